"""xz filter chains on the device: what undoing an x86 BCJ or a delta filter costs beside the LZMA2 decode of the same
blocks, from the profile ranges xz_decode and xz_unfilter of la_gpu_xz_decode.

    python tools/measure_xz_chains.py [--blocks 64] [--unit 8] [--preset 6] [--reps 3] [--out FILE]

The input is the Python executable repeated to `unit` MiB, cut into blocks of 1 MiB, every block coded by liblzma with
the chain [x86, LZMA2] and with [delta(4), LZMA2] and a CRC64 behind it, tiled in HBM to `blocks` blocks.  Every status
has to be OK and the first and last tile's bytes are compared with the plain bytes on the device.  For x86 the lengths
of the segments one lane walks (head to next head, la_xz_filters_dev.h) are counted on the host."""
import argparse
import lzma
import os
import statistics
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def segment_histogram(filtered):
    """lengths of the runs of E8 / E9 bytes less than 6 apart (one lane's serial walk), as {upper bound: count}"""
    a = np.frombuffer(filtered, dtype=np.uint8)
    ops = np.flatnonzero((a & 0xFE) == 0xE8)
    if ops.size == 0:
        return {}, 0
    cuts = np.flatnonzero(np.diff(ops) > 5)
    starts = np.concatenate([[0], cuts + 1])
    ends = np.concatenate([cuts, [ops.size - 1]])
    lens = ops[ends] - ops[starts] + 1
    hist = {}
    for bound in (1, 8, 32, 128, 512, 4096, 1 << 30):
        hist[bound] = int((lens <= bound).sum()) - sum(hist.values())
    return hist, int(lens.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--unit", type=int, default=8)
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
    say("# tools/measure_xz_chains.py --blocks %d --unit %d --preset %d --reps %d" % (args.blocks, args.unit, args.preset, args.reps))
    with open(sys.executable, "rb") as f:
        exe = f.read()
    plain = (exe * ((args.unit << 20) // len(exe) + 1))[:args.unit << 20]
    parts = [plain[i:i + (1 << 20)] for i in range(0, len(plain), 1 << 20)]
    tiles = max(args.blocks // len(parts), 1)
    lz = {"id": lzma.FILTER_LZMA2, "preset": args.preset}
    dict_size = lzma._decode_filter_properties(lzma.FILTER_LZMA2, lzma._encode_filter_properties(lz))["dict_size"]
    for name, chain, front in (("x86", [(4, 0)], {"id": lzma.FILTER_X86}), ("delta(4)", [(3, 4)], {"id": lzma.FILTER_DELTA, "dist": 4})):
        raws = [lzma.compress(p, format=lzma.FORMAT_RAW, filters=[front, lz]) for p in parts]
        if name == "x86":
            hist, longest = segment_histogram(lzma.decompress(raws[0], format=lzma.FORMAT_RAW, filters=[lz]))
            say("x86, first block: segments by length " + ", ".join("<=%d: %d" % kv for kv in hist.items() if kv[0] < 1 << 30) +
                ", longer: %d; the longest %d bytes" % (hist[1 << 30], longest))
        unit_img, unit_entries, dst = b"", [], 0
        for p, r in zip(parts, raws):
            unit_entries.append((len(unit_img), len(r), len(p), dst))
            unit_img += r + bytes(-len(r) % 4) + struct.pack("<Q", XB.crc64(p))
            dst += len(p)
        entries = [{"src_off": k * len(unit_img) + so, "comp_size": cs, "uncomp_size": us, "dst_off": k * len(plain) + do, "dst_cap": us,
                    "check_id": 4, "dict_size": dict_size} for k in range(tiles) for so, cs, us, do in unit_entries]
        total = tiles * len(plain)
        ctx = la.GpuContext(0)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.profile_enable(True)
        d_src = torch.from_numpy(np.frombuffer(unit_img, dtype=np.uint8).copy()).cuda().repeat(tiles)
        d_plain = torch.from_numpy(np.frombuffer(plain, dtype=np.uint8).copy()).cuda()
        plan = X.XzDevicePlan(ctx, d_src, X.block_table(entries), dst_cap=total, chains=[chain] * len(entries))
        decode, unfilter = [], []
        for rep in range(args.reps + 1):    # the first call warms the workspace and the code objects
            plan.run()
            ctx.sync()
            phases = dict(ctx.profile_read())
            if rep:
                decode.append(phases["xz_decode"])
                unfilter.append(phases["xz_unfilter"])
        res = plan.results()
        assert (res["status"] == 0).all(), res["status"][res["status"] != 0][:8]
        assert torch.equal(plan.d_dst[:len(plain)], d_plain) and torch.equal(plan.d_dst[total - len(plain):total], d_plain)
        d, u = statistics.median(decode), statistics.median(unfilter)
        say("[%s, LZMA2], %d blocks of 1 MiB (ratio %.2f), checks verified, median of %d calls: xz_decode %.1f ms, xz_unfilter %.3f ms (%.2f %% of the decode; %.0f MiB/s)"
            % (name, len(entries), len(plain) / len(unit_img), len(decode), d, u, 100.0 * u / d, total / 2 ** 20 / (u / 1e3)))
        ctx.close()
        del d_src, d_plain, plan
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
