"""bzip2 read side on the device: rate and time per phase, resident in HBM and through la_cat, against libbz2 on one
host core.

    python tools/measure_bzip2.py [--mib 1024] [--unit 64] [--levels 9,1] [--out FILE] [--no-cat]

Two inputs, C2-like (the bench's synthetic lz4 corpus, plain side) and text-like (random words), each compressed by
Python's bz2 (libbz2) as ONE stream per `unit` MiB and tiled to `mib` MiB (concatenated streams, what `cat a.bz2 b.bz2`
gives).  Resident: the image lies in HBM, one scan, then measure + emit over as many candidates as the workspace slots
(la_gpu_bzip2_max_blocks), the stream state carried from call to call; the output of every call is compared with the
plain bytes.  Phases are la_gpu_profile_read's, summed over the calls."""
import argparse
import bz2
import os
import subprocess
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--unit", type=int, default=64)
    ap.add_argument("--levels", default="9,1")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-cat", action="store_true")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    import torch
    import libarchive_amd as la
    from libarchive_amd import bzip2 as B
    say("# tools/measure_bzip2.py --mib %d --unit %d --levels %s" % (args.mib, args.unit, args.levels))
    reps = max(args.mib // args.unit, 1)
    for name, gen in (("c2_like", c2_like), ("text_like", text_like)):
        plain = gen(args.unit)
        for level in [int(x) for x in args.levels.split(",")]:
            t = time.time()
            unit_img = bz2.compress(plain, level)
            t_comp = time.time() - t
            t = time.time()
            assert bz2.decompress(unit_img) == plain
            t_host = time.time() - t
            img = unit_img * reps
            total = len(plain) * reps
            say("%s level %d: %d MiB plain, %.1f MiB compressed (ratio %.2f); libbz2 on one core: %.1f MiB/s decoded (compress %.1f s per unit)"
                % (name, level, total >> 20, len(img) / 2 ** 20, total / len(img), len(plain) / 2 ** 20 / t_host, t_comp))
            ctx = la.GpuContext(0)
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            ctx.profile_enable(True)
            d_src = torch.from_numpy(np.frombuffer(img, dtype=np.uint8).copy()).cuda()
            d_plain = torch.from_numpy(np.frombuffer(plain, dtype=np.uint8).copy()).cuda()
            for rep in range(2):        # the first pass warms the allocator and the workspace
                phases = {}
                ctx.timer_start()
                cands = B.scan(ctx, d_src, cap=1 << 18)
                for k, v in ctx.profile_read():
                    phases[k] = phases.get(k, 0.0) + v
                max_n = B.max_blocks(level)
                state, i0, done, calls, ok = None, 0, 0, 0, True
                while i0 < len(cands):
                    plan = B.Bz2DevicePlan(ctx, d_src, cands[i0:i0 + max_n], slot_level=level, state=state)
                    plan.measure()
                    for k, v in ctx.profile_read():
                        phases[k] = phases.get(k, 0.0) + v
                    st = plan.emit()
                    for k, v in ctx.profile_read():
                        phases[k] = phases.get(k, 0.0) + v
                    calls += 1
                    n_out = int(st["total_out"])
                    if rep == 1 and n_out:      # compare on the device: every call's bytes against the tiled plain text
                        off = done % len(plain)
                        got = plan.d_dst[:n_out]
                        idx = (torch.arange(n_out, device=got.device) + off) % len(plain)
                        ok = ok and bool(torch.equal(got, d_plain[idx]))
                    done += n_out
                    if int(st["first_bad"]) != 0xFFFFFFFF or int(st["n_taken"]) == 0:
                        ok = False
                        break
                    i0 += int(st["n_taken"])
                    state = {"open": int(st["open"]), "level": int(st["level"]), "crc": int(st["crc"]), "start_bit": int(st["start_bit"])}
                ms = ctx.timer_stop()
            assert ok and done == total, (ok, done, total)
            say("  resident in HBM: %d candidates, %d decode calls, %.1f ms wall (with the harness's allocations and read-backs) = %.0f MiB/s decoded; kernels %.1f ms = %.0f MiB/s"
                % (len(cands), calls, ms, total / 2 ** 20 / (ms / 1e3), sum(phases.values()), total / 2 ** 20 / (sum(phases.values()) / 1e3)))
            say("  phases (ms): " + ", ".join("%s %.1f" % kv for kv in sorted(phases.items(), key=lambda kv: -kv[1])))
            ctx.close()
            del d_src, d_plain
            if not args.no_cat:
                with tempfile.NamedTemporaryFile(suffix=".bz2", delete=False) as f:
                    f.write(img)
                t = time.time()
                run = subprocess.run([os.path.join(ROOT, "libarchive_amd", "host", "la_cat"), f.name], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
                dt = time.time() - t
                os.unlink(f.name)
                say("  la_cat: rc %d, %.2f s = %.0f MiB/s decoded (process start, device open, windows of LA_GPU_BATCH_MIB)%s"
                    % (run.returncode, dt, total / 2 ** 20 / dt, "" if run.returncode == 0 else " " + run.stderr.decode()[-200:]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
