"""lzip read side on the device: la_gpu_lzip_scan and la_gpu_lzip_decode on members resident in HBM, CRC32 verified,
against liblzma's raw LZMA1 decoder (Python's lzma) on one host core of the same machine over the same members.

    python tools/measure_lzip.py [--mib 256] [--unit 16] [--members 64,1024,16384] [--preset 6] [--reps 2] [--out FILE]

Two inputs, word text and the bench stream's kind of data (tests/streams.synth_lz4_stream's plain bytes), `unit` MiB
each, cut into members of 64 KiB, 1 MiB and 16 MiB of input (16 MiB is what plzip -6 writes), every piece one complete
member (header, LZMA stream with its end marker, 20-byte trailer), the unit tiled in HBM to `mib` MiB.  The scan runs
over the whole image and is timed on its own; its candidates are chained on the host by the trailers' member sizes, as
the filter does, and have to give exactly the members that were written.  One la_gpu_lzip_decode call then takes the
whole table with the trailers' ends, sizes and CRCs.  One warm-up call, then `reps` calls timed with events on the
context's stream: the median is reported.  Every status has to be OK and the first and last tile's bytes are compared
with the plain text on the device."""
import argparse
import lzma
import os
import statistics
import struct
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

DICT_BYTE = 23      # 8 MiB, the dictionary of lzip -6


def inputs(mib):
    import deflate_find_support as F
    import streams as S
    n = mib << 20
    frames = max(1, n // (16 * 65536))
    synth = S.synth_lz4_stream(0x4C413335, 0, frames, blocks_per_frame=16, block_size=65536, nthreads=8)[1].tobytes()[:n]
    return (("word text", F.word_text(n, seed=41)), ("bench-stream data", synth))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--unit", type=int, default=16)
    ap.add_argument("--members", default="64,1024,16384", help="member sizes in KiB of input")
    ap.add_argument("--preset", type=int, default=6)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    import torch
    import libarchive_amd as la
    from libarchive_amd import lzip as L
    say("# tools/measure_lzip.py --mib %d --unit %d --members %s --preset %d --reps %d" % (args.mib, args.unit, args.members, args.preset, args.reps))
    tiles = max((args.mib + args.unit - 1) // args.unit, 1)
    filt = [{"id": lzma.FILTER_LZMA1, "preset": args.preset, "lc": 3, "lp": 0, "pb": 2, "dict_size": 1 << DICT_BYTE}]
    for name, plain in inputs(args.unit):
        for ms in [int(x) << 10 for x in args.members.split(",")]:
            parts = [plain[i:i + ms] for i in range(0, len(plain), ms)]
            t = time.time()
            raws = [lzma.compress(p, format=lzma.FORMAT_RAW, filters=filt) for p in parts]
            t_comp = time.time() - t
            t = time.time()
            for p, r in zip(parts, raws):
                d = lzma.LZMADecompressor(format=lzma.FORMAT_RAW, filters=filt)
                assert d.decompress(r) == p and d.eof
            t_host = time.time() - t
            unit_img, unit_entries, dst = b"", [], 0
            for p, r in zip(parts, raws):
                m = b"LZIP\x01" + bytes([DICT_BYTE]) + r + struct.pack("<IQQ", zlib.crc32(p), len(p), 6 + len(r) + 20)
                unit_entries.append((len(unit_img), len(m), len(p), dst, zlib.crc32(p)))
                unit_img += m
                dst += len(p)
            entries = [{"src_off": k * len(unit_img) + so + 6, "src_end": k * len(unit_img) + so + ml - 20, "data_size": us,
                        "dst_off": k * len(plain) + do, "dst_cap": us, "dict_size": L.dict_size(DICT_BYTE), "crc32": crc}
                       for k in range(tiles) for so, ml, us, do, crc in unit_entries]
            total = tiles * len(plain)
            say("%s, members of %d KiB: %d MiB plain in %d members, %.1f MiB compressed (ratio %.2f); liblzma on one core: %.1f MiB/s decoded (compress %.1f s per unit)"
                % (name, ms >> 10, total >> 20, len(entries), tiles * len(unit_img) / 2 ** 20, len(plain) / len(unit_img), len(plain) / 2 ** 20 / t_host, t_comp))
            ctx = la.GpuContext(0)
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            d_unit = torch.from_numpy(np.frombuffer(unit_img, dtype=np.uint8).copy()).cuda()
            d_src = d_unit.repeat(tiles)
            d_plain = torch.from_numpy(np.frombuffer(plain, dtype=np.uint8).copy()).cuda()
            # the scan, and the chain the host builds from it
            scan_ms = []
            for rep in range(args.reps + 1):
                ctx.timer_start()
                offs, count = L.scan(ctx, d_src, cap=1 << 20)
                t_ms = ctx.timer_stop()
                if rep:
                    scan_ms.append(t_ms)
            img_len = tiles * len(unit_img)
            img = unit_img * tiles
            cands = [int(o) for o in offs] + [img_len]
            starts, s, ci = [], 0, 0
            while s < img_len:
                starts.append(s)
                while cands[ci] <= s:
                    ci += 1
                k = ci
                while struct.unpack_from("<Q", img, cands[k] - 8)[0] != cands[k] - s:
                    k += 1
                s = cands[k]
            assert [s + 6 for s in starts] == [e["src_off"] for e in entries], "the chain of candidates is not the members written"
            say("  scan of %.1f MiB: median %.2f ms = %.0f GiB/s, %d candidates for %d members"
                % (img_len / 2 ** 20, statistics.median(scan_ms), img_len / 2 ** 30 / (statistics.median(scan_ms) / 1e3), count, len(entries)))
            plan = L.LzipDevicePlan(ctx, d_src, L.member_table(entries), dst_cap=total)
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
            say("  resident in HBM, CRC32 verified: median of %d calls %.1f ms (min %.1f, max %.1f) = %.0f MiB/s decoded"
                % (len(times), med, min(times), max(times), total / 2 ** 20 / (med / 1e3)))
            ctx.close()
            del d_src, d_unit, d_plain, plan
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
